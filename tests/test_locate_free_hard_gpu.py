"""The free-aspect rescoring on the GPU, sum by sum (ssw_locate_free_sums_rgb8: the stage of ssw_locate_free_rgb8 from a start
the test gives, every sum returned) on the hard cases of tests/locate_free_cases.py: tie-heavy and saturated frames, starts on
every edge of the frame, suspects that reach the tiles listed in test_locate_free_hard_cpu.RESIZE_TILES.  The WHOLE array
must EQUAL the one built from the numpy restatement (locate_free_ref(..., start=..., details=True)) -- every scored slot, all ones everywhere else -- and the
answer the restatement's and, where the content decides it (locate_free_cases.truth, confirmed by
tests/test_locate_free_hard_cpu.py), that answer.  Integers, no tolerance, no case left out."""
import ctypes as C
import tempfile

import numpy as np
import pytest

import gpu_util as G
import locate_free_cases as FC
import spread_spectrum_watermarking_amd as wm
from spread_spectrum_watermarking_amd import _lib as L
from spread_spectrum_watermarking_amd.api import Locate
from test_locate_free_cpu import locate_free_ref
from test_locate_scale_cpu import with_alpha

pytestmark = pytest.mark.gpu


def sums_call(ctx, base, s, start, wmin, wmax, a, offset=0):
    """-> (status, sums [(2a + 1)^2][81] u64, (pw, ph, x, y, sad)); offset: the suspect lies that many bytes into its allocation."""
    H, W = base.shape[:2]
    db = ctx.to_device(base)
    ds = ctx.to_device(np.concatenate([np.zeros(offset, np.uint8), s.reshape(-1)]))
    sums = np.zeros(((2 * min(a, 4) + 1) ** 2, FC.SIDE * FC.SIDE), np.uint64)                # a above 4 is refused: nothing is written
    pl, sad = L.Placement(), C.c_uint64(7)
    rc = G.lib().ssw_locate_free_sums_rgb8(ctx.handle, db.ptr, W, H, C.c_void_p(ds.ptr.value + offset), s.shape[1], s.shape[0], s.shape[2],
                                           (C.c_uint32 * 4)(*start[:4]), wmin, wmax, a, sums.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(pl), C.byref(sad))
    for b in (db, ds):
        b.free()
    if rc == L.SSW_OK:
        assert (pl.w, pl.h, pl.channels) == (s.shape[1], s.shape[0], s.shape[2])
    return rc, sums, (pl.pw, pl.ph, pl.x, pl.y, sad.value)


def run(name, ctx=None, offset=0):
    c = FC.BY_NAME[name]
    base, s = FC.pixels(name)
    rc, sums, answer = sums_call(ctx or G.ctx(), base, s, c.start, c.wmin, c.wmax, c.slack, offset)
    assert rc == L.SSW_OK, rc
    return sums, answer


def tile_of(c, pw, ph):
    """The tile of one item, for a failure's report (the host program is built only then)."""
    try:
        it = [(p, q) for p, q, _ in FC.items(c)].index((pw, ph))
        with tempfile.TemporaryDirectory() as d:
            return FC.tiles(FC.build_plan_program(d), [c])[c.name][it]
    except Exception as e:                                                          # the report must not hide the mismatch
        return "tile unknown (%s)" % type(e).__name__


def assert_sums_equal(c, start, a, got, want, what=""):
    if np.array_equal(got, want):
        return
    s, p = (int(v[0]) for v in np.nonzero(got != want))
    pw, ph, x, y = FC.candidate(start, a, s, p)
    n = int((got != want).sum())
    pytest.fail("%s %s: %d of %d slots differ; the first at (pw, ph, x, y) = %s: gpu %d, numpy %d; %s"
                % (c.name, what, n, got.size, (pw, ph, x, y), int(got[s, p]), int(want[s, p]), tile_of(c, pw, ph)))


def check(name, got, answer, what=""):
    c = FC.BY_NAME[name]
    want, want_answer = FC.reference(name)
    assert_sums_equal(c, c.start, c.slack, got, want, what)
    assert answer == want_answer, (name, what)
    truth = FC.truth(c)
    if truth is not None:
        assert answer[:4] == truth[:4] and (truth[4] is None or answer[4] == truth[4]), (name, what)


@pytest.mark.parametrize("name", FC.names())
def test_every_sum_equals_the_restatement(name):
    """Tables T (tile edges), W (windows and the frame's edge) and X (contents): the whole host_sums array."""
    got, answer = run(name)
    print(name, "answer", answer, "scored", int((got != FC.EMPTY).sum()))
    check(name, got, answer)


@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("name", ["X plain noise", "X resized binary"])
def test_suspect_pointers_of_every_alignment(name, off):
    """Three channels, the suspect 1, 2 and 3 bytes into its allocation: one case per front."""
    assert FC.BY_NAME[name].channels == 3
    got, answer = run(name, offset=off)
    check(name, got, answer, "suspect at +%d" % off)


PUBLIC = ["X plain flat", "X plain rows", "X resized noise", "X resized periodic", "X rgba binary", "X rgba columns"]


def found(f):
    return (f.placement.w, f.placement.h, f.placement.x, f.placement.y, f.sad)


@pytest.mark.parametrize("name", PUBLIC)
def test_the_public_call_answers_what_the_diagnostic_answers_from_the_ladders_start(name):
    """ssw_locate_free_rgb8 = the ladder, then the stage: its answer is the diagnostic's when that is started from what
    ssw_locate_scaled_rgb8 answers, and both are the restatement's without a start (its own ladder), the array included."""
    c = FC.BY_NAME[name]
    base, s = FC.pixels(name)
    want, a0, scores = locate_free_ref(base, s, c.wmin, c.wmax, c.slack, details=True)
    ladder = found(wm.locate(base, [s], [Locate(widths=(c.wmin, c.wmax))], ctx=G.ctx())[0])
    free = found(wm.locate(base, [s], [Locate(widths=(c.wmin, c.wmax), aspect=c.slack)], ctx=G.ctx())[0])
    rc, sums, answer = sums_call(G.ctx(), base, s, ladder, c.wmin, c.wmax, c.slack)
    print(name, "ladder", ladder, "numpy", a0, "free", free, "diagnostic", answer, "numpy", want)
    assert rc == L.SSW_OK and ladder == tuple(a0) and free == answer == want
    assert_sums_equal(c, a0, c.slack, sums, FC.sums_array(a0, c.slack, scores), "from the ladder's start")


def test_a_large_call_leaves_nothing_behind_for_a_small_one():
    """The case with the most tiles (81 sizes of 128 x 128, every slot of the sums' workspace written), then the one with a single
    size and a single position, on one context: every slot as a fresh context gives it."""
    big, small = "T 128x128 x0.95 rgba noise", "W 160x32 one size, one position"
    ctx = G.ctx()
    check(big, *run(big, ctx))
    after = run(small, ctx)
    with G.fresh_ctx() as fresh:
        alone = run(small, fresh)
    assert np.array_equal(after[0], alone[0]) and after[1] == alone[1]
    assert int((after[0] != FC.EMPTY).sum()) == 1
    check(small, *after)


def test_five_hard_suspects_in_one_public_call():
    """Both fronts, three and four channels, a flat suspect among them (every candidate of its ladder and of its stage ties or
    nearly so): 25 + 25 + 49 + 81 + 9 items, split over launches by front and channel count.  Each as when it is alone."""
    base = FC.pixels("X plain noise")[0]
    three = ["X plain noise", "X resized noise", "X rgba noise"]
    assert all(np.array_equal(FC.pixels(n)[0], base) for n in three)
    sus = [FC.pixels(n)[1] for n in three]
    entries = [Locate(widths=(FC.BY_NAME[n].wmin, FC.BY_NAME[n].wmax), aspect=FC.BY_NAME[n].slack) for n in three]
    sus.append(np.full((36, 40, 3), 131, np.uint8)); entries.append(Locate(widths=(36, 48), aspect=4))                    # flat, the plain front
    x, y, pw, ph = FC.BY_NAME["X resized noise"].rect
    sus.append(with_alpha(FC.LC.noisy(FC.LC.cut(base, x, y, pw, ph), 3), 9)); entries.append(Locate(widths=(56, 72), aspect=1))   # RGBA at its own size
    together = wm.locate(base, sus, entries, ctx=G.ctx())
    for i, (s, e, g) in enumerate(zip(sus, entries, together)):
        alone = wm.locate(base, [s], [e], ctx=G.ctx())[0]
        print(i, s.shape, "together", found(g), "alone", found(alone))
        assert found(g) == found(alone), i
    for n, g in zip(three, together):                                              # exact and resized cuts of noise: the truth
        assert found(g)[:4] == FC.truth(FC.BY_NAME[n])[:4], n
    assert found(together[4])[:4] == (pw, ph, x, y)


def test_status_codes_of_the_diagnostic():
    lib, ctx = G.lib(), G.ctx()
    c = FC.BY_NAME["X rgba noise"]
    base, s = FC.pixels(c.name)
    H, W = base.shape[:2]
    sh, sw, ch = s.shape
    pw0, ph0, x0, y0 = c.start
    call = lambda start=c.start, lo=c.wmin, hi=c.wmax, a=c.slack: sums_call(ctx, base, s, start, lo, hi, a)[0]
    assert call() == L.SSW_OK
    for a in (0, 5, 81, 0xFFFFFFFF):
        assert call(a=a) == L.SSW_ERR_BAD_ARG, a
    assert call(lo=50, hi=49) == L.SSW_ERR_BAD_ARG                               # wmin > wmax
    for bad in ((0, ph0, x0, y0), (pw0, 0, x0, y0), (W + 1, ph0, 0, y0), (pw0, H + 1, x0, 0), (pw0, ph0, W - pw0 + 1, y0), (pw0, ph0, x0, H - ph0 + 1),
                (pw0, ph0, 0xFFFFFFFF, y0)):
        assert call(start=bad) == L.SSW_ERR_BAD_ARG, bad
    assert call(start=(W, H, 0, 0), lo=32, hi=W) == L.SSW_OK                      # the whole frame is a start
    # nothing scored at all: the range lies outside pw0 +- a -> all ones, the start and 0
    rc, sums, answer = sums_call(ctx, base, s, c.start, pw0 + 5, pw0 + 9, 3)
    assert rc == L.SSW_OK and np.all(sums == FC.EMPTY) and answer == c.start + (0,)
    # wmin below 32 is not the diagnostic's business: sizes stop at 32
    rc, sums, answer = sums_call(ctx, base, s, (33, 33, 5, 5), 1, 40, 2)
    assert rc == L.SSW_OK and int((sums != FC.EMPTY).any(axis=1).sum()) == 16     # 32 .. 35 in both dimensions
    db, ds = ctx.to_device(base), ctx.to_device(s)
    out, pl, sad, st = (C.c_uint64 * (49 * 81))(), L.Placement(), C.c_uint64(), (C.c_uint32 * 4)(*c.start)
    full = [ctx.handle, db.ptr, W, H, ds.ptr, sw, sh, ch, st, c.wmin, c.wmax, c.slack, out, C.byref(pl), C.byref(sad)]
    assert lib.ssw_locate_free_sums_rgb8(*full) == L.SSW_OK
    for k in (0, 1, 4, 8, 12, 13, 14):                                             # every pointer
        args = list(full)
        args[k] = None
        assert lib.ssw_locate_free_sums_rgb8(*args) == L.SSW_ERR_BAD_ARG, k
    for k, v in ((7, 2), (7, 5), (5, 0), (6, 0), (2, 0), (3, 0)):                  # channels, a zero size
        args = list(full)
        args[k] = v
        assert lib.ssw_locate_free_sums_rgb8(*args) == L.SSW_ERR_BAD_ARG, (k, v)
    for b in (db, ds):
        b.free()
