"""ssw_locate_turned_rgb8 on the GPU against the restatement of tests/test_locate_turned_cpu.py: EQUALITY -- the answer's n, x, y,
tw, th and sad and every rung's (D, n_j, x, y) -- on the eight cases of the cat (against the recorded answers) and at the smallest
shapes at which the kernels can go wrong: sides that are no multiple of 4, one rung, the largest angles, a strip whose upper rungs
are dropped, a suspect of the original's size, one wider than the original, ties at every stage, noise, and a call whose launches
are cut at 32 items.  The template kernel's box means are compared on their own."""
import ctypes as C
import io
import math

import numpy as np
import pytest

import locate_cases as LC
from gpu_util import ctx, lib
from spread_spectrum_watermarking_amd import _lib as L
from PIL import Image
from spread_spectrum_watermarking_amd import api, cli
from spread_spectrum_watermarking_amd._lib import SswError, check
from test_angle_cpu import rungs_ref, smooth, turned
from test_locate_cpu import luma
from test_locate_turned_cpu import (CASES, SEARCH, boxes_ref, cat, locate_turned_ref, name_of, recorded, restore_turned_ref, template_ref,
                                    template_size_ref, true_centre, turned_cut)

pytestmark = pytest.mark.gpu


class Dev:
    def __init__(self, a):
        a = np.ascontiguousarray(a)
        self.buf = ctx().alloc(a.nbytes + 16)
        check(lib().ssw_copy_to_dev(ctx().handle, self.buf.ptr, a.ctypes.data, a.nbytes), "ssw_copy_to_dev")

    @property
    def ptr(self):
        return self.buf.ptr

    def free(self):
        self.buf.free()


def dev_locate(base, suspects, amin, amax, want_rungs=True, channels=3):
    """-> ([(n, x, y, tw, th, sad)] per suspect, rungs [n][n_rungs][4]) of one call"""
    n = len(suspects)
    b, dev = Dev(base), [Dev(s) for s in suspects]
    ptrs = (C.c_void_p * n)(*[d.ptr.value for d in dev])
    shapes = (L.TurnedShape * n)(*[L.TurnedShape(s.shape[1], s.shape[0], channels) for s in suspects])
    found = (L.TurnedFound * n)()
    j0, j1 = rungs_ref(amin, amax) if math.isfinite(amin) and math.isfinite(amax) and amin <= amax else (0, 0)      # (a refused range: any buffer)
    rungs = np.full((n, j1 - j0 + 1, 4), 0xA5A5A5A5, np.uint64)
    try:
        check(lib().ssw_locate_turned_rgb8(ctx().handle, b.ptr, base.shape[1], base.shape[0], ptrs, shapes, n, amin, amax, found,
                                           rungs.ctypes.data if want_rungs else None), "ssw_locate_turned_rgb8")
    finally:
        for d in dev + [b]:
            d.free()
    assert all(f.n_rungs == j1 - j0 + 1 for f in found)
    return [(f.n, f.x, f.y, f.tw, f.th, f.sad) for f in found], rungs


def same(got, rungs, want_answers, want_rungs, what):
    for i, (g, a, r) in enumerate(zip(got, want_answers, want_rungs)):
        want = np.asarray(r, np.uint64)
        bad = np.nonzero((rungs[i] != want).any(axis=1))[0]
        assert bad.size == 0, (what, i, "rung", int(bad[0]), rungs[i][bad[0]].tolist(), r[bad[0]])
        assert g == tuple(a), (what, i, g, tuple(a))


def same_as_ref(base, suspects, amin, amax, what):
    got, rungs = dev_locate(base, suspects, amin, amax)
    refs = [locate_turned_ref(base, s, amin, amax) for s in suspects]
    same(got, rungs, [r.answer() for r in refs], [r.rung_rows() for r in refs], what)
    return refs


def cut(frame, x, y, w, h):
    return np.ascontiguousarray(frame[y:y + h, x:x + w])


# ---- the photograph -----------------------------------------------------------------------------------------------------------
def test_the_eight_cat_cases_equal_the_recorded_answers():
    base, marked = cat()
    rec = recorded()
    got, rungs = dev_locate(base, [turned_cut(marked, *c) for c in CASES], *SEARCH)
    same(got, rungs, [rec[name_of(c)]["answer"] for c in CASES], [rec[name_of(c)]["rungs"] for c in CASES], "cat")


def test_the_python_surface_on_a_cat_case():
    base, marked = cat()
    c = CASES[5]
    rec = recorded()[name_of(c)]
    (f,), entries = api.locate_turned(base, [turned_cut(marked, *c)], SEARCH, ctx(), rungs=True)
    n, x, y, tw, th, sad = rec["answer"]
    assert (f.n, f.angle, f.centre, f.template, f.sad) == (n, n / 32, (x + tw / 2.0, y + th / 2.0), (tw, th), sad)
    assert f.mean_abs_diff == sad / (tw * th) and entries.tolist() == [rec["rungs"]]
    assert api.locate_turned(base, [], SEARCH, ctx()) == []
    with pytest.raises(ValueError):                                     # the translation search does not take such an entry silently
        api.locate(base, [turned_cut(marked, *c)], [api.Locate(turned=True)], ctx())


# ---- small shapes -------------------------------------------------------------------------------------------------------------
def test_64x64_and_70x66_in_96x80():
    base = smooth(96, 80)
    t = turned(base, 2.1)
    same_as_ref(base, [cut(t, 20, 10, 64, 64), cut(t, 13, 7, 70, 66)], -4, 4, "96x80")


def test_no_side_a_multiple_of_4():
    base = smooth(101, 83)
    same_as_ref(base, [cut(turned(base, -3.0), 17, 9, 67, 65)], -5, 5, "101x83")


def test_a_range_of_one_rung():
    base = smooth(96, 80)
    r = same_as_ref(base, [cut(turned(base, 1.0), 16, 8, 64, 64)], 1.0, 1.0, "one rung")[0]
    assert (r.j0, r.j1, r.kept) == (4, 4, [0]) and r.n == 32


def test_the_largest_angles_on_64x64():
    base = smooth(96, 80)
    s = [cut(turned(base, 44.0), 16, 8, 64, 64), cut(turned(base, -45.0), 16, 8, 64, 64)]
    refs = same_as_ref(base, s, -45, 45, "+-45")
    assert refs[0].n_rungs == 361 and template_size_ref(64, 64, 1440) == (40, 40) and refs[0].rungs[0][4:] == (40, 40) and refs[0].rungs[-1][4:] == (40, 40)


def test_a_strip_whose_upper_rungs_are_dropped():
    base = smooth(1040, 80)
    r = same_as_ref(base, [cut(turned(base, 1.25), 20, 8, 1000, 64)], 0, 10, "strip")[0]
    assert r.rungs[0] is not None and r.rungs[-1] is None and r.rung_rows()[-1] == [0, 0, 0, 0]


def test_every_rung_dropped_is_bad_dims():
    base = smooth(1040, 80)
    for s, lo, hi in ((cut(base, 20, 8, 1000, 64), 10, 12), (cut(base, 0, 0, 30, 30), -1, 1), (np.zeros((200, 1048, 3), np.uint8), -1, 1)):
        with pytest.raises(SswError) as e:
            dev_locate(base, [s], lo, hi)
        assert e.value.status == L.SSW_ERR_BAD_DIMS


def test_a_suspect_of_the_originals_size():
    base = smooth(96, 80)
    same_as_ref(base, [turned(base, 2.0), base], -3, 3, "own size")


def test_templates_that_do_not_fit_the_frame_at_small_angles():
    base = smooth(96, 80)
    wide = smooth(112, 60, seed=3)                                      # wider than the original: only a turned-back part of it fits
    r = same_as_ref(base, [wide], 0, 25, "wide")[0]
    assert r.rungs[0] is None and r.rungs[-1] is not None


def test_a_flat_frame_ties_at_every_stage():
    flat = np.full((80, 96, 3), 93, np.uint8)
    r = same_as_ref(flat, [flat[:64, :64]], -1, 1, "flat")[0]
    assert r.kept == [0, 1, 2, 3] and (r.n, r.x, r.y, r.sad) == (-32, 0, 0, 0)


def test_noise():
    base = np.random.default_rng(64).integers(0, 256, (80, 96, 3), dtype=np.uint8)
    same_as_ref(base, [cut(turned(base, 1.5), 10, 5, 70, 66), cut(base, 3, 2, 64, 64)], -2, 2, "noise")


@pytest.mark.parametrize("content", LC.LADDER_CONTENTS)
def test_tied_contents(content):
    W, H = LC.LADDER_BASE
    base = LC.frame(content, H, W, seed=ord("T"))
    same_as_ref(base, [cut(base, 93, 51, 129, 65), LC.noisy(cut(base, 40, 30, 80, 72), 1)], -0.5, 0.5, content)


def test_nine_suspects_of_mixed_sizes_cut_a_launch_at_32_items():
    base = smooth(160, 120)
    sizes = [(64, 64), (70, 66), (67, 65), (96, 40), (40, 96), (128, 100), (81, 49), (56, 72), (100, 100)]
    s = [cut(turned(base, a), 5 + i, 3 + i, w, h) for i, ((w, h), a) in enumerate(zip(sizes, (3.3, -7.9, 0.7, 9.6, 0.0, 1.0, -2.5, 5.0, -9.9)))]
    refs = same_as_ref(base, s, -10, 10, "nine")
    assert all(r.n_rungs == 81 for r in refs)


# ---- the template kernel on its own ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sw,sh", [(70, 66), (333, 251)])
@pytest.mark.parametrize("n", [-1440, 7, 424])
def test_rung_boxes_equal_the_restatements(sw, sh, n):
    s = np.random.default_rng([sw, n + 1440]).integers(0, 256, (sh, sw, 3), dtype=np.uint8)
    tw, th = template_size_ref(sw, sh, n)
    d = Dev(s)
    gw, gh = C.c_uint32(0), C.c_uint32(0)
    got = np.full((th // 8, tw // 8), 0xA5, np.uint8)
    try:
        check(lib().ssw_locate_turned_rung_boxes(ctx().handle, d.ptr, sw, sh, n, C.byref(gw), C.byref(gh), got.ctypes.data), "ssw_locate_turned_rung_boxes")
    finally:
        d.free()
    assert (gw.value, gh.value) == (tw, th)
    assert (got == boxes_ref(template_ref(luma(s), n, tw, th))).all()


# ---- errors ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    base = smooth(96, 80)
    s = cut(base, 0, 0, 64, 64)
    for lo, hi in ((2, 1), (-46, 0), (0, 45.5), (float("nan"), 1), (0, float("inf"))):
        with pytest.raises(SswError) as e:
            dev_locate(base, [s], lo, hi)
        assert e.value.status == L.SSW_ERR_BAD_ARG
    with pytest.raises(SswError) as e:
        dev_locate(base, [np.zeros((64, 64, 4), np.uint8)], -1, 1, channels=4)
    assert e.value.status == L.SSW_ERR_UNSUPPORTED
    with pytest.raises(SswError) as e:
        dev_locate(base, [s], -1, 1, channels=2)
    assert e.value.status == L.SSW_ERR_BAD_ARG
    found = (L.TurnedFound * 1)()
    assert lib().ssw_locate_turned_rgb8(ctx().handle, None, 96, 80, None, None, 0, 5.0, 1.0, None, None) == 0           # n == 0 first
    assert lib().ssw_locate_turned_rgb8(ctx().handle, None, 96, 80, None, None, 1, -1.0, 1.0, found, None) == L.SSW_ERR_BAD_ARG


# ---- restoring --------------------------------------------------------------------------------------------------------------------
def dev_restore(base, suspects, triples):
    return api.restore_turned(base, suspects, triples, ctx())


def test_tiny_suspects_give_the_original_back():
    """1 x 1 holds no footprint: the mask is empty.  5 x 4 holds the footprints of x = 1, 2 at y = 1: whatever the restatement keeps"""
    base = smooth(96, 80)
    rng = np.random.default_rng(9)
    one, five = rng.integers(0, 256, (1, 1, 3), dtype=np.uint8), rng.integers(0, 256, (4, 5, 3), dtype=np.uint8)
    got = dev_restore(base, [one, five, five], [(0.0, 40.5, 30.5), (0.0, 40.5, 30.0), (3.0, 17.25, 60.5)])
    assert (got[0] == base).all()
    for g, s, t in zip(got[1:], (five, five), ((0.0, 40.5, 30.0), (3.0, 17.25, 60.5))):
        assert (g == restore_turned_ref(base, s, *t)).all()


@pytest.mark.parametrize("angle", [0.0, 0.03125, -7.9, 30.0, 45.0])
def test_64x64_in_96x80_at_five_angles(angle):
    base = smooth(96, 80)
    s = cut(turned(smooth(96, 80, seed=1), angle), 16, 8, 64, 64)
    (got,) = dev_restore(base, [s], [(angle, 48.0, 40.0)])
    want = restore_turned_ref(base, s, angle, 48.0, 40.0)
    assert (got == want).all() and (want != base).any()


def test_a_centre_given_in_fractions_and_a_cut_out_past_the_border():
    base = smooth(101, 83)
    s = [smooth(67, 65, seed=2), smooth(70, 66, seed=3), smooth(64, 64, seed=4)]
    t = [(3.3, 50.37, 41.81), (-12.0, 5.0, 3.5), (8.0, 99.0, 90.25)]   # the last two reach past the original's border
    for g, si, ti in zip(dev_restore(base, s, t), s, t):
        want = restore_turned_ref(base, si, *ti)
        assert (g == want).all() and (want != base).any() and (want == base).any()


def test_restore_argument_errors():
    base = smooth(96, 80)
    b, d = Dev(base), Dev(np.zeros((64, 64, 3), np.uint8))
    out = ctx().alloc(96 * 80 * 3)
    ptrs = (C.c_void_p * 1)(d.ptr.value)
    job = (L.TurnedJob * 1)(L.TurnedJob(1.0, 48.0, 40.0))
    call = lambda shape, jb=job, base_ptr=b.ptr, o=out.ptr, n=1: lib().ssw_restore_turned_rgb8(ctx().handle, base_ptr, 96, 80, ptrs, (L.TurnedShape * 1)(shape), jb, n, o)
    try:
        assert call(L.TurnedShape(64, 64, 3)) == 0
        assert call(L.TurnedShape(64, 64, 3), n=0, base_ptr=None) == 0
        assert call(L.TurnedShape(64, 64, 3), base_ptr=None) == L.SSW_ERR_BAD_ARG
        assert call(L.TurnedShape(64, 64, 3), (L.TurnedJob * 1)(L.TurnedJob(float("nan"), 1.0, 1.0))) == L.SSW_ERR_BAD_ARG
        assert call(L.TurnedShape(64, 64, 2)) == L.SSW_ERR_BAD_ARG
        assert call(L.TurnedShape(64, 64, 4)) == L.SSW_ERR_UNSUPPORTED
        assert call(L.TurnedShape(0, 64, 3)) == L.SSW_ERR_BAD_DIMS and call(L.TurnedShape(64, 65536, 3)) == L.SSW_ERR_BAD_DIMS
        assert call(L.TurnedShape(64, 64, 3), o=b.ptr) == L.SSW_ERR_BAD_ARG                # the output overlaps the original
    finally:
        b.free(); d.free(); out.free()


# ---- end to end -----------------------------------------------------------------------------------------------------------------
# How far a copy's own similarity may fall below the one of the restoration with the TRUE angle and centre (the yardstick).  The
# search answers on a grid of 1/32 degree and half a pixel, so what it restores lies a fraction of a pixel beside the yardstick's
# frame.  Measured on an MI355X, own mark / yardstick: 16.36 / 16.46 (a loss of 0.6 %), 12.10 / 15.17 (20.2 % -- the
# case the search answers 4.2/32 degree and 0.45 pixels from the truth) and 21.66 / 21.87 (1.0 %).  The inputs and the search are
# deterministic (integers); only the trace's f32 sums (1e-4 relative) can move these figures.  The bound is 1.5 times the worst
# loss measured, so that it fails when a change costs the worst case another half of what the grid already costs it.
OWN_MARK_MAY_LOSE = 0.30


def test_turned_cut_outs_are_traced_to_their_copies():
    import spread_spectrum_watermarking_amd as wm
    base, _ = cat()
    k = 1000
    marks = np.random.default_rng(11).standard_normal((3, k)).astype(np.float32)
    copies = wm.Writer(base, wm.WriteConfig(), ctx()).mark_copies_rgb8(list(marks))
    cases = CASES[:3]
    sus = [turned_cut(np.asarray(c), *case) for c, case in zip(copies, cases)]
    ctx().reset_timing(); ctx().enable_timing(True)
    res = wm.trace_many(base, sus, list(marks), ctx=ctx(), placements=[wm.Locate(turned=True)] * 3)
    ctx().synchronize()
    t = ctx().timing()
    ctx().enable_timing(False)
    assert t["locate"]["launches"] > 0 and t["locate_coarse"]["launches"] > 0 and t["resize"]["launches"] > 0
    assert list(res.best) == [0, 1, 2] and sorted(res.located_turned) == [0, 1, 2]
    found = [res.located_turned[i] for i in range(3)]
    assert found == wm.locate_turned(base, sus, ctx=ctx())
    frames = wm.restore_turned(base, sus, found, ctx())
    assert all((a == b).all() for a, b in zip(wm.restore(base, sus, [wm.Locate(turned=True)] * 3, ctx()), frames))      # `restore` says what is traced
    again = wm.trace_many(base, frames, list(marks), ctx=ctx())
    assert (again.sims == res.sims).all() and (again.extracted == res.extracted).all() and (again.best_sim == res.best_sim).all()
    H, W = base.shape[:2]
    truth = [(case[0],) + tuple(v / 2.0 for v in true_centre(W, H, *case)) for case in cases]
    yard = wm.trace_many(base, wm.restore_turned(base, sus, truth, ctx()), list(marks), ctx=ctx())
    for i in range(3):
        own, want = float(res.sims[i, i]), float(yard.sims[i, i])
        print("copy", i, "found", found[i].angle, found[i].centre, "truth", truth[i], "own mark", own, "yardstick", want, "loss", 1.0 - own / want)
        assert own > 6.0 and want > 6.0
        assert own >= (1.0 - OWN_MARK_MAY_LOSE) * want


def test_no_turned_search_without_turned_entries():
    import spread_spectrum_watermarking_amd as wm
    base, _ = cat()
    marks = np.random.default_rng(3).standard_normal((2, 200)).astype(np.float32)
    copies = wm.Writer(base, wm.WriteConfig(), ctx()).mark_copies_rgb8(list(marks))
    c = cut(np.asarray(copies[1]), 160, 60, 400, 320)
    ctx().reset_timing(); ctx().enable_timing(True)
    res = wm.trace_many(base, [copies[0], c], list(marks), ctx=ctx(), placements=[None, wm.Placement(160, 60)])
    ctx().synchronize()
    t = ctx().timing()
    assert t["locate"]["launches"] == 0 and t["locate_coarse"]["launches"] == 0 and res.located_turned == {}
    ctx().reset_timing()
    res = wm.trace_many(base, [copies[0], c], list(marks), ctx=ctx(), placements=[None, wm.Locate()])
    ctx().synchronize()
    t = ctx().timing()
    ctx().enable_timing(False)
    assert t["locate_coarse"]["launches"] == 1 and res.located_turned == {} and list(res.best) == [0, 1]      # today's one search, no ladder


def test_cli_records_carry_the_centre_and_the_angle(tmp_path):
    """fingerprint two copies of the cat, turn and crop them with Pillow, trace them with --locate FILE=rotate:? and its kin"""
    base, _ = cat()
    Image.fromarray(base).save(tmp_path / "base.png")
    assert cli.main(["fingerprint", str(tmp_path / "base.png"), "--copies", "2", "-d", "copy"]) == 0
    copies = [np.asarray(Image.open(tmp_path / f"base_fp{i}.png").convert("RGB")) for i in range(2)]
    names = [str(tmp_path / f"cut{i}.png") for i in range(2)]
    for name, c, case in zip(names, copies, (CASES[0], CASES[4])):
        Image.fromarray(turned_cut(c, *case)).save(name)
    out = io.StringIO()
    args = cli.build_parser().parse_args(["trace", str(tmp_path / "base.png"), "--suspects", *names, "--marks", str(tmp_path / "base_fp.json"),
                                          "--locate", f"{names[0]}=rotate:?", "--locate", f"{names[1]}=rotate:-1..1"])
    assert cli.cmd_trace(args, out) == 0
    text = out.getvalue()
    assert text.count("  Matches: true") == 2, text
    assert '  Located: "centre 319.0,240.0 turned 3.3125 (mean luma difference ' in text and '  Located: "centre 361.0,221.0 turned 0 (mean luma difference ' in text, text
    assert "turned back by 3.3125 degrees about 319.0,240.0, completed with the base" in text, text
