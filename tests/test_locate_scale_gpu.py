"""Locating cut-outs of unknown scale on the GPU (ssw_locate_scaled_rgb8): pw, ph, x, y and SAD must EQUAL the numpy
restatement of the scale ladder (tests/test_locate_scale_cpu.py: locate_scaled_ref, whose answers are recorded in
tests/golden/locate_scale_answers.json and checked against the restatement by the CPU tests) -- everything is an integer,
there is no tolerance -- and tracing with `Locate(widths=...)` entries must give, bit for bit, what tracing with the
placements it found gives."""
import ctypes as C

import numpy as np
import pytest

import gpu_util as G
import spread_spectrum_watermarking_amd as wm
from oracle import oracle as O
from spread_spectrum_watermarking_amd import _lib as L
from spread_spectrum_watermarking_amd.api import Locate, Placement
from test_locate_cpu import cat, cut, luma
from test_locate_scale_cpu import EXTRA, SIX, box8, case, recorded, with_alpha

pytestmark = pytest.mark.gpu

FIELDS = ("extracted", "sims", "best", "best_sim", "n_exceed")


def answer(f):
    return (f.placement.w, f.placement.h, f.placement.x, f.placement.y, f.sad)


@pytest.mark.parametrize("name", list(SIX) + EXTRA)
def test_equals_the_restatement(name):
    base, s, lo, hi, _ = case(name)
    got = wm.locate(base, [s], [Locate(widths=(lo, hi))], ctx=G.ctx())[0]
    want = recorded()[name]
    print(name, "gpu", answer(got), "numpy", want)
    assert answer(got) == want and got.size == want[:2] and got.mean_abs_diff == got.sad / (want[0] * want[1])
    if name == "rgba":
        assert answer(got) == recorded()["narrow rgb"]
    if name.startswith("one width"):                                    # the true position lies in the kept window: today's search at that size
        assert answer(wm.locate(base, [s], [Locate(400, 320)], ctx=G.ctx())[0]) == want
    if name == "401x321 unscaled":
        assert Locate(scale=(350 / 401, 450 / 401)).width_range(401) == (350, 450)
        assert answer(wm.locate(base, [s], [Locate(scale=(350 / 401, 450 / 401))], ctx=G.ctx())[0]) == want


def test_nine_suspects_with_different_ranges_in_one_call():
    """154 (suspect, rung) items: five launches of descriptors; sized and unsized entries ride along in their own call."""
    names = list(SIX) + ["rgba", "wmin at 32", "pw/8 leaves 7"]
    cases = [case(n) for n in names]
    base = cases[0][0]
    sus = [c[1] for c in cases] + [cut(cat()[1], 301, 150, 70, 66)]
    entries = [Locate(widths=(c[2], c[3])) for c in cases] + [Locate()]
    got = wm.locate(base, sus, entries, ctx=G.ctx())
    for n, g in zip(names, got):
        print(n, "gpu", answer(g), "numpy", recorded()[n])
    assert [answer(g) for g in got[:9]] == [recorded()[n] for n in names]
    assert (got[9].placement.x, got[9].placement.y, got[9].size) == (301, 150, (70, 66))


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("pw,ph", [(400, 320), (393, 314), (151, 121)], ids=["doubled", "odd", "reduced"])
def test_rung_boxes_equal_the_box_means_of_the_restored_frame(pw, ph, channels):
    """T_j of locate_rung_kernel against ssw_restore_rgb8's resize of the same suspect: luma, then 8 x 8 box means, bit for bit."""
    lib, ctx = G.lib(), G.ctx()
    half = O.resize_rgb8(cut(cat()[1], 161, 61, 400, 320), 200, 160)
    s = with_alpha(half, 7) if channels == 4 else half                  # the rung kernel ignores alpha ...
    opaque = np.ascontiguousarray(np.concatenate([half, np.full(half.shape[:2] + (1,), 255, np.uint8)], 2)) if channels == 4 else half
    frame = wm.restore(np.zeros((ph, pw, 3), np.uint8), [opaque], [Placement(0, 0, pw, ph)], ctx=ctx)[0]   # ... the restore blends it: opaque there
    want = box8(luma(frame))[::8, ::8][:ph // 8, :pw // 8]
    ds = ctx.to_device(s)
    got = np.zeros((ph // 8, pw // 8), np.uint8)
    rc = lib.ssw_locate_rung_boxes(ctx.handle, ds.ptr, 200, 160, channels, pw, ph, got.ctypes.data)
    ds.free()
    assert rc == L.SSW_OK
    assert want.shape == got.shape and np.array_equal(got, want), np.abs(got.astype(int) - want).max()


# The rung kernel on the shared front end of the fused tile (csrc/resize_common.hpp) at its edges; what pick_resize_tile chooses
# for each shape, printed from a scratch build, is in the comment.  (suspect w, h, channels, rung w, h, bytes the suspect's
# pointer is offset by)
RUNG_TILE_CASES = [
    (505, 487, 3, 64, 56, 1),    # rows of 1515 B behind an odd pointer: tile 8 x 16, 4-word vertical pieces
    (505, 487, 4, 64, 56, 0),    # tile 8 x 8, 2-word vertical pieces
    (211, 173, 3, 417, 341, 0),  # rows of 633 B: tile 32 x 128 over the 416 x 336 pixels that lie in a box, last tile 16 x 32
    (211, 173, 4, 300, 250, 1),  # tile 32 x 128 of 69248 B of LDS (> 64 KB), last tile 24 x 40
]


@pytest.mark.parametrize("sw,sh,c,pw,ph,off", RUNG_TILE_CASES)
def test_rung_boxes_at_the_tile_edges(sw, sh, c, pw, ph, off):
    """As above: T_j against the box means of the restored frame, bit for bit."""
    lib, ctx = G.lib(), G.ctx()
    s = np.random.default_rng(sw + c).integers(0, 256, (sh, sw, c), dtype=np.uint8)
    opaque = s.copy()
    opaque[..., 3:] = 255                                               # the rung kernel ignores alpha, the restore blends it
    frame = wm.restore(np.zeros((ph, pw, 3), np.uint8), [opaque], [Placement(0, 0, pw, ph)], ctx=ctx)[0]
    want = box8(luma(frame))[::8, ::8][:ph // 8, :pw // 8]
    ds = ctx.to_device(np.concatenate([np.zeros(off, np.uint8), s.reshape(-1)]))
    got = np.zeros((ph // 8, pw // 8), np.uint8)
    rc = lib.ssw_locate_rung_boxes(ctx.handle, C.c_void_p(ds.ptr.value + off), sw, sh, c, pw, ph, got.ctypes.data)
    ds.free()
    assert rc == L.SSW_OK
    assert want.shape == got.shape and np.array_equal(got, want), np.abs(got.astype(int) - want).max()


def test_three_half_scale_cut_outs_name_their_copies():
    base, _ = cat()
    k = 1000
    marks = np.random.default_rng(5).standard_normal((3, k)).astype(np.float32)
    ctx = G.ctx()
    copies = wm.Writer(base, wm.WriteConfig(), ctx).mark_copies_rgb8(list(marks))
    rects = [(160, 60, 400, 320), (100, 40, 480, 360), (120, 50, 440, 340)]
    sus = [O.resize_rgb8(cut(c, *r), r[2] // 2, r[3] // 2) for c, r in zip(copies, rects)]
    loc = [Locate(widths=(360, 520)), Locate(widths=(400, 560)), Locate(scale=(1.6, 2.4))]
    found = wm.locate(base, sus, loc, ctx=ctx)
    print("located", [(f.placement, round(f.mean_abs_diff, 3)) for f in found])
    print("truth  ", rects)
    got = wm.trace_many(base, sus, list(marks), ctx=ctx, placements=loc)
    ref = wm.trace_many(base, sus, list(marks), ctx=ctx, placements=[f.placement for f in found])
    for name in FIELDS:
        assert np.array_equal(getattr(got, name), getattr(ref, name), equal_nan=True), name
    print("best", got.best, "best_sim", got.best_sim)
    for j in range(3):
        assert got.best[j] == j and got.best_sim[j] > 6.0 and got.n_exceed[j] == 1, (j, got.best, got.best_sim, got.n_exceed)


def test_a_call_without_ranged_entries_launches_nothing_new():
    base, marked = cat()
    ctx = G.ctx()
    half = O.resize_rgb8(cut(marked, 161, 61, 400, 320), 200, 160)
    ctx.reset_timing(); ctx.enable_timing(True)
    wm.locate(base, [cut(marked, 161, 61, 400, 320)], [Locate()], ctx=ctx)
    ctx.synchronize()
    t = ctx.timing()
    assert t["locate_coarse"]["launches"] == 1 and t["resize"]["launches"] == 0, t      # no rung tile, no second coarse search
    ctx.reset_timing()
    wm.locate(base, [half], [Locate(400, 320)], ctx=ctx)
    ctx.synchronize()
    t = ctx.timing()
    assert t["locate_coarse"]["launches"] == 1 and t["resize"]["launches"] == 1, t
    ctx.reset_timing()
    wm.locate(base, [half], [Locate(widths=(384, 416))], ctx=ctx)
    ctx.synchronize()
    t = ctx.timing()
    ctx.enable_timing(False)
    assert t["locate_coarse"]["launches"] > 1 and t["resize"]["launches"] > 1 and t["locate"]["ms"] > 0.0, t


def test_status_codes():
    lib, ctx = G.lib(), G.ctx()
    base, marked = cat()
    H, W = base.shape[:2]
    s = with_alpha(O.resize_rgb8(cut(marked, 161, 61, 400, 320), 200, 160), 1)
    db, ds = ctx.to_device(base), ctx.to_device(s)
    ptrs = (C.c_void_p * 1)(ds.ptr.value)
    sad = (C.c_uint64 * 1)()
    P = lambda *a: (L.Placement * 1)(L.Placement(*a))
    R = lambda lo, hi: (L.ScaleRange * 1)(L.ScaleRange(lo, hi))
    call = lambda pl, rg, n=1: lib.ssw_locate_scaled_rgb8(ctx.handle, db.ptr, W, H, ptrs, pl, rg, n, sad)
    pl = P(200, 160, 4, 77, 99, 5, 6)                                 # x, y, pw, ph are outputs: what is there is not read
    assert call(pl, R(392, 408)) == L.SSW_OK and (pl[0].pw, pl[0].ph, pl[0].x, pl[0].y, sad[0]) == recorded()["narrow rgb"]
    assert call(P(200, 160, 4, 0, 0, 0, 0), R(408, 392)) == L.SSW_ERR_BAD_ARG          # wmin > wmax
    assert call(P(200, 160, 4, 0, 0, 0, 0), R(31, 100)) == L.SSW_ERR_BAD_ARG           # under 32
    assert call(P(200, 160, 4, 0, 0, 0, 0), R(39, 100)) == L.SSW_ERR_BAD_ARG           # ph(39) = 31
    assert call(P(200, 160, 4, 0, 0, 0, 0), R(641, 700)) == L.SSW_ERR_BAD_ARG          # no rung fits the frame
    assert call(P(200, 160, 4, 0, 0, 0, 0), R(560, 700)) == L.SSW_ERR_BAD_ARG          # ... 560 wide is 448 tall
    for ch in (0, 1, 2, 5):
        assert call(P(200, 160, ch, 0, 0, 0, 0), R(392, 408)) == L.SSW_ERR_BAD_ARG
    assert call(P(0, 160, 4, 0, 0, 0, 0), R(392, 408)) == L.SSW_ERR_BAD_ARG and call(P(200, 0, 4, 0, 0, 0, 0), R(392, 408)) == L.SSW_ERR_BAD_ARG
    assert call(P(9, 9, 9, 0, 0, 0, 0), R(9, 1), 0) == L.SSW_OK                        # n == 0
    assert lib.ssw_locate_scaled_rgb8(ctx.handle, db.ptr, W, H, ptrs, P(200, 160, 4, 0, 0, 0, 0), None, 1, sad) == L.SSW_ERR_BAD_ARG
    assert lib.ssw_locate_scaled_rgb8(ctx.handle, db.ptr, W, H, ptrs, P(200, 160, 4, 0, 0, 0, 0), R(392, 408), 1, None) == L.SSW_ERR_BAD_ARG
    assert lib.ssw_locate_scaled_rgb8(ctx.handle, None, W, H, ptrs, P(200, 160, 4, 0, 0, 0, 0), R(392, 408), 1, sad) == L.SSW_ERR_BAD_ARG
    with pytest.raises(ValueError):
        wm.locate(base, [s], [Locate(widths=(500, 400))], ctx=ctx)
    for b in (db, ds):
        b.free()
