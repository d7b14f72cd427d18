"""Locating scaled cut-outs whose aspect ratio was not kept exactly on the GPU (ssw_locate_free_rgb8): pw, ph, x, y and SAD must
EQUAL the numpy restatement (tests/test_locate_free_cpu.py: locate_free_ref, whose answers are recorded in
tests/golden/locate_free_answers.json and checked against the restatement by the CPU tests) -- everything is an integer, there
is no tolerance -- and tracing the 240 x 166 thumbnail with `Locate(widths=..., aspect=2)` must give the similarity of the
placed piece."""
import ctypes as C
import json

import numpy as np
import pytest

import gpu_util as G
import spread_spectrum_watermarking_amd as wm
from spread_spectrum_watermarking_amd import _lib as L
from spread_spectrum_watermarking_amd import api
from spread_spectrum_watermarking_amd.api import Locate
from test_locate_free_cpu import ALL, case, crop_thumb, recorded, slacks
from test_locate_scale_cpu import EXTRA, SIX
from test_locate_scale_cpu import recorded as scale_recorded

pytestmark = pytest.mark.gpu


def answer(f):
    return (f.placement.w, f.placement.h, f.placement.x, f.placement.y, f.sad)


def free(base, s, lo, hi, a):
    return wm.locate(base, [s], [Locate(widths=(lo, hi), aspect=a)], ctx=G.ctx())[0]


@pytest.mark.parametrize("name", ALL)
def test_equals_the_restatement(name):
    """Every recorded case: the crop thumbnails (480 x 333 at 80,55 found exactly), the off-aspect pieces (a = 4: 81 sizes,
    three launches), the corner piece (windows clipped at W - pw, H - ph; sizes that leave the frame), 34 x 34 (sizes clipped
    at 32), enlargements of 3 (RGB), 0.95 (RGB) and 1.2 (RGBA) -- where the cheapest resize tile leaves no LDS for the window
    and the tile is chosen with it counted --, and the ladder's own fifteen -- RGBA, the piece at 3,5 (window clipped at 0), wmin == wmax, the 40 x 40 piece at
    wmin 32, an unscaled suspect (R = S is one of the sizes); every case meets widths with pw mod 4 = 0, 1, 2 and 3."""
    base, s, lo, hi, _ = case(name)
    for a in slacks(name):
        ladder, want = recorded()[name][a]
        got = free(base, s, lo, hi, a)
        print(name, "a", a, "gpu", answer(got), "numpy", want, "ladder", ladder)
        assert answer(got) == want and got.size == want[:2] and got.mean_abs_diff == got.sad / (want[0] * want[1])
        assert answer(wm.locate(base, [s], [Locate(widths=(lo, hi))], ctx=G.ctx())[0]) == ladder
    if name == "rgba":
        assert recorded()[name] == recorded()["narrow rgb"]


FIVE = [("400x320 -> 203x160", 4), ("corner 300x200 -> 151x100", 2), ("rgba", 1), ("34x34 unscaled", 4), ("401x321 unscaled", 3)]


def test_five_suspects_of_different_sizes_and_slacks_in_one_call():
    """81 + 25 + 9 + 49 + 49 = 213 (suspect, size) items, resized and not, three and four channels: seven launches of descriptors.
    Against the same suspects one per call, and against the record where it has the slack."""
    cases = [case(n) for n, _ in FIVE]
    base = cases[0][0]
    got = wm.locate(base, [c[1] for c in cases], [Locate(widths=(c[2], c[3]), aspect=a) for c, (_, a) in zip(cases, FIVE)], ctx=G.ctx())
    for (n, a), c, g in zip(FIVE, cases, got):
        assert np.array_equal(c[0], base)
        alone = free(c[0], c[1], c[2], c[3], a)
        print(n, "a", a, "together", answer(g), "alone", answer(alone))
        assert answer(g) == answer(alone)
        if a in recorded()[n]:
            assert answer(g) == recorded()[n][a][1]
    # entries of every kind side by side: each group in its own call, the answers in the caller's order
    mixed = wm.locate(base, [cases[0][1], cases[2][1], cases[4][1]], [Locate(widths=(300, 500), aspect=4), Locate(widths=(384, 416)), Locate()], ctx=G.ctx())
    assert answer(mixed[0]) == recorded()[FIVE[0][0]][4][1] and answer(mixed[1]) == scale_recorded()["rgba"]
    assert (mixed[2].placement.x, mixed[2].placement.y, mixed[2].size) == (161, 61, (401, 321))


def test_the_thumbnail_is_traced_at_the_placed_similarity():
    """480 x 333 at 80,55 of copy 0 (alpha 0.02), halved by Pillow to 240 x 166: with aspect=2 the trace names the copy with the
    similarity of the piece laid where it belongs, without it with the similarity of the ladder's answer one row off --
    both figures from tests/golden/crop_answers.json (the CPU oracle's), to their two decimals."""
    from conftest import GOLDEN
    from test_crop_cpu import marks
    from test_jpeg_cpu import cat_image
    import os
    with open(os.path.join(GOLDEN, "crop_answers.json")) as f:
        rec = json.load(f)["scaled"]["80,55,480x333->240x166"]["0.02"]
    base, thumb, ctx = cat_image(), crop_thumb(166, 0, 0.02), G.ctx()
    cfg = api.ReadConfig(extraction=api.Extraction.Option2(0.02))
    sims = {}
    for what, entry in (("free", Locate(widths=(240, 640), aspect=2)), ("ladder", Locate(widths=(240, 640)))):
        res = wm.trace_many(base, [thumb], list(marks()), threshold=6.0, config=cfg, ctx=ctx, placements=[entry])
        sims[what] = float(np.asarray(res.sims, np.float64)[0][0])
        print(what, "similarity", sims[what], "best", res.best[0], "recorded placed / found", rec["sim_placed"], rec["sim_found"])
        assert res.best[0] == 0
    assert round(sims["free"], 2) == rec["sim_placed"] == 16.02
    assert round(sims["ladder"], 2) == rec["sim_found"] == 6.68


def test_the_ladder_answers_as_before_after_the_new_call():
    """ssw_locate_scaled_rgb8 on a context the new call just used: the recorded answers of locate_scale_answers.json, whatever
    the stage left in the workspace it shares (luma plane, tap tables)."""
    ctx = G.ctx()
    for name in ("400x320 halved", "rgba", "164x128 doubled", "401x321 unscaled", "wmin at 32", "pw/8 leaves 7"):
        base, s, lo, hi, _ = case(name)
        free(base, s, lo, hi, 4)
        got = wm.locate(base, [s], [Locate(widths=(lo, hi))], ctx=ctx)[0]
        assert answer(got) == scale_recorded()[name], name
    assert set(SIX) | set(EXTRA) == set(scale_recorded())


def test_the_stage_is_billed_to_resize_and_locate():
    base, s, lo, hi, _ = case("407x326 -> 203x163")
    ctx = G.ctx()
    ctx.reset_timing(); ctx.enable_timing(True)
    wm.locate(base, [s], [Locate(widths=(lo, hi))], ctx=ctx)
    ctx.synchronize()
    before = ctx.timing()
    ctx.reset_timing()
    free(base, s, lo, hi, 2)
    ctx.synchronize()
    t = ctx.timing()
    ctx.enable_timing(False)
    assert t["resize"]["launches"] == before["resize"]["launches"] + 1 and t["locate"]["launches"] == before["locate"]["launches"] + 1, (before, t)
    assert t["locate_coarse"]["launches"] == before["locate_coarse"]["launches"] and len(L.STAGES) == 15


def test_status_codes():
    lib, ctx = G.lib(), G.ctx()
    base, s, lo, hi, _ = case("rgba")
    H, W = base.shape[:2]
    db, ds = ctx.to_device(base), ctx.to_device(s)
    ptrs = (C.c_void_p * 1)(ds.ptr.value)
    sad = (C.c_uint64 * 1)()
    P = lambda *a: (L.Placement * 1)(L.Placement(*a))
    R = lambda lo, hi: (L.ScaleRange * 1)(L.ScaleRange(lo, hi))
    A = lambda a: (C.c_uint32 * 1)(a)
    call = lambda pl, rg, sl, n=1: lib.ssw_locate_free_rgb8(ctx.handle, db.ptr, W, H, ptrs, pl, rg, sl, n, sad)
    pl = P(200, 160, 4, 77, 99, 5, 6)                                 # x, y, pw, ph are outputs: what is there is not read
    assert call(pl, R(lo, hi), A(2)) == L.SSW_OK and (pl[0].pw, pl[0].ph, pl[0].x, pl[0].y, sad[0]) == recorded()["rgba"][2][1]
    for a in (0, 5, 81, 0xFFFFFFFF):
        assert call(P(200, 160, 4, 0, 0, 0, 0), R(lo, hi), A(a)) == L.SSW_ERR_BAD_ARG
    assert call(P(200, 160, 4, 0, 0, 0, 0), R(408, 392), A(2)) == L.SSW_ERR_BAD_ARG       # the ladder's codes pass through: wmin > wmax
    assert call(P(200, 160, 4, 0, 0, 0, 0), R(31, 100), A(2)) == L.SSW_ERR_BAD_ARG        # under 32
    assert call(P(200, 160, 4, 0, 0, 0, 0), R(641, 700), A(2)) == L.SSW_ERR_BAD_ARG       # no rung fits the frame
    assert call(P(200, 160, 5, 0, 0, 0, 0), R(lo, hi), A(2)) == L.SSW_ERR_BAD_ARG
    assert call(P(9, 9, 9, 0, 0, 0, 0), R(9, 1), A(9), 0) == L.SSW_OK                     # n == 0
    assert call(P(200, 160, 4, 0, 0, 0, 0), R(lo, hi), None) == L.SSW_ERR_BAD_ARG
    assert call(P(200, 160, 4, 0, 0, 0, 0), None, A(2)) == L.SSW_ERR_BAD_ARG
    assert lib.ssw_locate_free_rgb8(ctx.handle, None, W, H, ptrs, P(200, 160, 4, 0, 0, 0, 0), R(lo, hi), A(2), 1, sad) == L.SSW_ERR_BAD_ARG
    assert lib.ssw_locate_free_rgb8(ctx.handle, db.ptr, W, H, ptrs, P(200, 160, 4, 0, 0, 0, 0), R(lo, hi), A(2), 1, None) == L.SSW_ERR_BAD_ARG
    with pytest.raises(ValueError):
        wm.locate(base, [s], [Locate(widths=(lo, hi), aspect=5)], ctx=ctx)
    for b in (db, ds):
        b.free()
