"""Locating cut-outs of unknown scale (ssw_locate_scaled_rgb8): the parts that need no GPU -- the numpy restatement of the
scale ladder defined in include/ssw.h (the yardstick of tests/test_locate_scale_gpu.py, which imports it from here), what it
finds on the reference's photograph, the Python resolution of `Locate(widths=...)` / `Locate(scale=...)` entries and the
CLI's --locate FILE=W0..W1."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from oracle import oracle as O
from spread_spectrum_watermarking_amd import _lib as L
from spread_spectrum_watermarking_amd import api, cli
from test_locate_cpu import cat, cut, locate_ref, luma, restored

RUNG_STEP, STRIDE, BOX, KEEP, NEAR_W, NEAR_XY = 8, 4, 8, 8, 7, 8


# ---- the definition of include/ssw.h (ssw_locate_scaled_rgb8), restated -----------------------------------------------------------
def height_of(pw, sw, sh):
    return max(1, (2 * sh * pw + sw) // (2 * sw))


def box8(lum):
    """(sum of the 8 x 8 lumas at (x, y) + 32) >> 6 at every position where the box fits: [h - 7][w - 7]."""
    c = np.cumsum(np.cumsum(np.pad(lum, ((1, 0), (1, 0))), 0), 1)
    return (c[8:, 8:] - c[:-8, 8:] - c[8:, :-8] + c[:-8, :-8] + 32) >> 6


def rungs_of(W, H, sw, sh, wmin, wmax):
    """The widths of the ladder; ValueError is the C side's SSW_ERR_BAD_ARG."""
    if wmin > wmax or min(wmin, height_of(wmin, sw, sh)) < 32:
        raise ValueError("range")
    ws = list(range(wmin, wmax + 1, RUNG_STEP))
    if ws[-1] != wmax:
        ws.append(wmax)
    ws = [pw for pw in ws if pw <= W and height_of(pw, sw, sh) <= H]
    if not ws:
        raise ValueError("no rung fits the frame")
    return ws


def ladder(base, s, wmin, wmax):
    """Per rung (pw, ph, D, y, x, n): the smallest (D, y, x) of the rung's box search."""
    H, W = base.shape[:2]
    sh, sw = s.shape[:2]
    b8 = box8(luma(base))[::STRIDE, ::STRIDE]
    out = []
    for pw in rungs_of(W, H, sw, sh, wmin, wmax):
        ph = height_of(pw, sw, sh)
        t = box8(luma(restored(s, pw, ph)))[::BOX, ::BOX][:ph // BOX, :pw // BOX]
        nx, ny = (W - pw) // STRIDE + 1, (H - ph) // STRIDE + 1
        d = np.zeros((ny, nx), np.int64)
        for k in range(t.shape[0]):
            for i in range(t.shape[1]):
                d += np.abs(b8[2 * k:2 * k + ny, 2 * i:2 * i + nx] - t[k, i])
        idx = int(np.argmin(d.ravel()))                                # the first minimum in (y, x) order
        out.append((pw, ph, int(d.ravel()[idx]), STRIDE * (idx // nx), STRIDE * (idx % nx), t.size))
    return out


def kept_rungs(rungs):
    """The 8 rungs with the smallest D / n (cross-multiplied), ties to the smaller j."""
    import functools
    cmp = lambda a, b: (rungs[a][2] * rungs[b][5] > rungs[b][2] * rungs[a][5]) - (rungs[a][2] * rungs[b][5] < rungs[b][2] * rungs[a][5]) or a - b
    return sorted(range(len(rungs)), key=functools.cmp_to_key(cmp))[:KEEP]


def refine_jobs(rungs, keep, W, H, sw, sh, wmin, wmax):
    """(pw, ph, window) of every windowed search of the refinement, in the order (kept rung, width); identical ones once."""
    jobs = []
    for j in keep:
        pwj, _, _, yj, xj, _ = rungs[j]
        for pw in range(max(wmin, pwj - NEAR_W), min(wmax, pwj + NEAR_W) + 1):
            ph = height_of(pw, sw, sh)
            if pw > W or ph > H:
                continue
            win = (max(0, xj - NEAR_XY), min(W - pw, xj + NEAR_XY), max(0, yj - NEAR_XY), min(H - ph, yj + NEAR_XY))
            if win[0] <= win[1] and win[2] <= win[3] and (pw, ph, win) not in jobs:
                jobs.append((pw, ph, win))
    return jobs


def locate_scaled_ref(base, s, wmin, wmax, details=False):
    """-> (pw, ph, x, y, sad): the smallest sad / (pw ph), ties to the smaller pw, then y, then x."""
    H, W = base.shape[:2]
    sh, sw = s.shape[:2]
    rungs = ladder(base, s, wmin, wmax)
    keep = kept_rungs(rungs)
    resized, best = {}, None
    for pw, ph, win in refine_jobs(rungs, keep, W, H, sw, sh, wmin, wmax):
        if pw not in resized:
            resized[pw] = restored(s, pw, ph)
        x, y, sad = locate_ref(base, resized[pw], window=win)
        if best is None or (sad * best[0] * best[1], pw, y, x) < (best[4] * pw * ph, best[0], best[3], best[2]):
            best = (pw, ph, x, y, sad)
    return (best, rungs, keep) if details else best


# ---- the cases: name -> (base, suspect, wmin, wmax, truth or None) ----------------------------------------------------------------
SIX = {"400x320 halved": ((161, 61, 400, 320), (200, 160), (300, 500)),
       "400x320 at three quarters": ((161, 61, 400, 320), (300, 240), (200, 640)),
       "600x430 halved": ((3, 5, 600, 430), (300, 215), (320, 640)),
       "164x128 halved": ((237, 93, 164, 128), (82, 64), (100, 300)),
       "164x128 doubled": ((237, 93, 164, 128), (328, 256), (100, 300)),
       "401x321 unscaled": ((161, 61, 401, 321), None, (350, 450))}


def with_alpha(rgb, seed):
    a = np.random.default_rng(seed).integers(0, 256, rgb.shape[:2] + (1,), dtype=np.uint8)
    return np.ascontiguousarray(np.concatenate([rgb, a], 2))


def case(name):
    base, marked = cat()
    if name in SIX:
        rect, size, rng = SIX[name]
        s = cut(marked, *rect)
        return base, (O.resize_rgb8(s, *size) if size else s), rng[0], rng[1], rect
    half = O.resize_rgb8(cut(marked, 161, 61, 400, 320), 200, 160)
    if name == "rgba":                                                  # the same answer as "narrow rgb"
        return base, with_alpha(half, 3), 384, 416, (161, 61, 400, 320)
    if name == "narrow rgb":
        return base, half, 384, 416, (161, 61, 400, 320)
    if name == "one width":
        return base, half, 400, 400, (161, 61, 400, 320)
    if name == "one width, unscaled":
        return base, cut(marked, 161, 61, 400, 320), 400, 400, (161, 61, 400, 320)
    if name == "wmin at 32":                                            # 41 x 32 quartered from 164 x 128: ph(32) = 25 < 32 is refused, a square works
        return base, cut(marked, 300, 150, 40, 40), 32, 56, (300, 150, 40, 40)
    if name == "upper rungs leave the frame":
        return base, O.resize_rgb8(cut(marked, 3, 5, 600, 430), 300, 215), 560, 900, (3, 5, 600, 430)
    if name == "637 wide":
        b, m = np.ascontiguousarray(base[:441, :637]), np.ascontiguousarray(marked[:441, :637])
        return b, O.resize_rgb8(cut(m, 161, 61, 400, 320), 200, 160), 380, 420, (161, 61, 400, 320)
    if name == "pw/8 leaves 1":                                         # every rung 8 j + 1 wide
        return base, O.resize_rgb8(cut(marked, 161, 61, 401, 321), 200, 160), 385, 417, (161, 61, 401, 321)
    if name == "pw/8 leaves 7":
        return base, O.resize_rgb8(cut(marked, 161, 61, 407, 326), 203, 163), 391, 423, (161, 61, 407, 326)
    raise KeyError(name)


EXTRA = ["rgba", "narrow rgb", "one width", "one width, unscaled", "wmin at 32", "upper rungs leave the frame", "637 wide",
         "pw/8 leaves 1", "pw/8 leaves 7"]
ANSWERS = os.path.join(GOLDEN, "locate_scale_answers.json")          # what the restatement answers, recorded: the GPU tests compare with it


def recorded():
    with open(ANSWERS) as f:
        return {k: tuple(v) for k, v in json.load(f).items()}


# ---- what it finds ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SIX))
def test_the_six_cases_are_found(name):
    """The first run of this search, with the constants of the issue (rung step 8, stride 4, box 8, 8 kept, +-7, +-8): all six
    are found exactly -- (pw, ph, x, y) equals the truth, offsets 0 -- so the halved-constants fallback was not needed."""
    base, s, lo, hi, (x, y, w, h) = case(name)
    best, rungs, keep = locate_scaled_ref(base, s, lo, hi, details=True)
    pw, ph, gx, gy, sad = best
    print(name, "->", best, "truth", (w, h, x, y), "offsets", (pw - w, ph - h, gx - x, gy - y), "mean", round(sad / (pw * ph), 3),
          "rungs", len(rungs), "kept", [rungs[j][0] for j in keep])
    if SIX[name][1] is None:
        assert (pw, ph, gx, gy) == (w, h, x, y)                         # an exact cut-out: the width lies on no rung
        assert sad == int(np.abs(luma(s) - luma(cut(base, x, y, w, h))).sum())
        assert all((w - r[0]) % RUNG_STEP for r in rungs)
    else:                                                               # a resized copy need not have its minimum at the exact integer width
        assert abs(pw - w) <= 1 and abs(gx - x) <= 1 and abs(gy - y) <= 1
    assert best == recorded()[name]


@pytest.mark.parametrize("name", EXTRA)
def test_the_recorded_answers_are_the_restatements(name):
    base, s, lo, hi, (x, y, w, h) = case(name)
    best = locate_scaled_ref(base, s, lo, hi)
    print(name, "->", best, "truth", (w, h, x, y))
    assert best == recorded()[name]
    if name == "rgba":
        assert best == recorded()["narrow rgb"]                         # alpha is ignored
    if name.startswith("one width"):                                    # one rung, one width: today's search in a window around the rung's entry
        r = restored(s, 400, 320)
        assert best == (400, 320) + locate_ref(base, r) and best[2:4] == (161, 61)


def test_rungs_and_argument_checks():
    assert rungs_of(640, 444, 200, 160, 300, 500) == list(range(300, 500, 8)) + [500]
    assert rungs_of(640, 444, 200, 160, 300, 316) == [300, 308, 316]                      # wmax hit: not added twice
    assert rungs_of(640, 444, 200, 160, 400, 400) == [400]
    assert rungs_of(640, 444, 300, 215, 560, 900)[-1] == 616 and height_of(616, 300, 215) == 441 and height_of(624, 300, 215) > 444
    assert rungs_of(640, 444, 40, 40, 32, 56) == [32, 40, 48, 56]
    assert height_of(401, 401, 321) == 321 and height_of(400, 200, 160) == 320 and height_of(1, 640, 1) == 1
    for bad in ((640, 444, 200, 160, 31, 500),      # wmin under 32
                (640, 444, 164, 128, 32, 200),      # ph(32) = 25
                (640, 444, 200, 160, 500, 300),     # wmin > wmax
                (640, 444, 200, 160, 648, 700),     # every rung wider than the frame
                (640, 444, 160, 200, 400, 500)):    # every rung taller than the frame
        with pytest.raises(ValueError):
            rungs_of(*bad)
    # ranking: D / n by cross-multiplication, ties to the smaller j
    rungs = [(0, 0, 10, 0, 0, 5), (0, 0, 4, 0, 0, 2), (0, 0, 3, 0, 0, 2), (0, 0, 20, 0, 0, 10)] + [(0, 0, 100, 0, 0, 1)] * 8
    assert kept_rungs(rungs) == [2, 0, 1, 3, 4, 5, 6, 7]


# ---- header, ABI ---------------------------------------------------------------------------------------------------------------
def test_header_states_the_ladder():
    text = open(os.path.join(ROOT, "include", "ssw.h")).read()
    assert text.index("ssw_locate_rgb8(ssw_ctx") < text.index("a scale ladder") < text.index("ssw_locate_scaled_rgb8(ssw_ctx")
    doc = text[text.index("a scale ladder"):text.index("ssw_locate_scaled_rgb8(ssw_ctx")]
    for phrase in ("pw_j = wmin + 8 j", "plus wmax if it was not hit", "max(1, (2 sh pw + sw) / (2 sw))", "+ 32) >> 6", "multiple\n   of 4".replace("\n   ", " "),
                   "smallest (D, y, x)", "D_a n_b against D_b n_a", "ties go to the\n       smaller j".replace("\n       ", " "), "[pw_j - 7, pw_j + 7]", "+-8",
                   "smallest SAD / (pw ph)", "ties: smaller pw, then y, then x", "aspect ratio is assumed kept", "no rotation",
                   "smooth regions are ambiguous", "min(pw, ph) >= 32", "min(wmin, ph(wmin)) < 32", "SSW_ERR_BAD_ARG", "SSW_ERR_UNSUPPORTED",
                   "n == 0: SSW_OK", "pw, ph, x, y of each placement are OUTPUTS", "waits for the stream twice", "SSW_STAGE_RESIZE"):
        assert phrase in " ".join(doc.split()), phrase
    assert len(L.SIGNATURES["ssw_locate_scaled_rgb8"][1]) == 9 and len(L.SIGNATURES["ssw_locate_rung_boxes"][1]) == 8
    assert [f[0] for f in L.ScaleRange._fields_] == ["wmin", "wmax"] and "SSW_STAGE_COUNT = 15" in text and len(L.STAGES) == 15


# ---- Python: ranged Locate entries --------------------------------------------------------------------------------------------------
def test_ranged_locate_entries():
    import spread_spectrum_watermarking_amd as wm
    assert api.Locate(widths=(300, 900)).width_range(200) == (300, 900)
    assert api.Locate(scale=(0.5, 2)).width_range(201) == (100, 402) and api.Locate(scale=(1.5, 1.5)).width_range(3) == (4, 5)
    assert api.Locate().width_range(200) is None and api.Locate(60, 50).width_range(200) is None
    assert api.Locate() == api.Locate(None, None, None, None) and api.Locate(60, 50) != api.Locate(widths=(60, 60))
    for bad in (api.Locate(widths=(5, 3)), api.Locate(widths=(0, 3)), api.Locate(widths=(3.5, 7)), api.Locate(scale=(0, 1)), api.Locate(scale=(2, 1)),
                api.Locate(60, 50, widths=(1, 2)), api.Locate(widths=(1, 2), scale=(1, 2))):
        with pytest.raises(ValueError):
            bad.width_range(100)
    f = api.Located(api.Placement(3, 5, 600, 430), 1000, 1000 / (600 * 430))
    assert f.size == (600, 430)
    # resolution: still ONE locate call, ranged and sized entries side by side
    base = np.zeros((444, 640, 3), np.uint8)
    sus = [np.zeros((50, 60, 3), np.uint8), np.zeros((160, 200, 3), np.uint8), np.zeros((25, 30, 4), np.uint8), np.zeros((8, 8, 3), np.uint8)]
    calls = []

    def fake(b, suspects, sizes, ctx):
        calls.append(([s.shape for s in suspects], list(sizes)))
        ranged = lambda z, s: z.width_range(s.shape[1]) is not None
        return [api.Located(api.Placement(10 + i, 20 + i, 400 if ranged(z, s) else (z.w or s.shape[1]), 320 if ranged(z, s) else (z.h or s.shape[0])), 100, 0.5)
                for i, (s, z) in enumerate(zip(suspects, sizes))]
    pls = [api.Locate(), api.Locate(widths=(300, 500)), api.Locate(scale=(1, 4)), api.Placement(1, 2)]
    out, found = api._resolve_locates(base, sus, pls, None, fake)
    assert len(calls) == 1 and calls[0][1] == pls[:3]
    assert out == [api.Placement(10, 20, 60, 50), api.Placement(11, 21, 400, 320), api.Placement(12, 22, 400, 320), api.Placement(1, 2)]
    assert sorted(found) == [0, 1, 2] and found[1].size == (400, 320)
    _, _, pl = api._placed_suspects(sus, out, 640, 444)
    assert [(p.x, p.y, p.pw, p.ph) for p in pl][1] == (11, 21, 400, 320)
    import inspect
    src = inspect.getsource(api.locate)
    assert "width_range" in src and "_locate_mixed" in src
    assert "ssw_locate_scaled_rgb8" in inspect.getsource(api._locate_mixed) and wm.Locate is api.Locate


# ---- CLI ---------------------------------------------------------------------------------------------------------------------
def test_locate_option_takes_a_range_of_widths():
    p = cli.build_parser()
    common = ["trace", "cat.jpg", "--suspects", "a.png", "b=c.png", "--marks", "x.json"]
    a = p.parse_args(common + ["--locate", "a.png=300..900"])
    assert a.locates == {"a.png": api.Locate(widths=(300, 900))}
    a = p.parse_args(common + ["--locate", "a.png=400x320", "--locate", "b=c.png=64..64"])
    assert a.locates == {"a.png": api.Locate(400, 320), "b=c.png": api.Locate(widths=(64, 64))}
    assert cli.parse_locate("a.png", ["a.png"]) == ("a.png", api.Locate()) and cli.parse_locate("a.png=4x5", ["a.png"]) == ("a.png", api.Locate(4, 5))
    for bad in ("a.png=300..", "a.png=..900", "a.png=..", "a.png=900..300", "a.png=0..5", "a.png=-3..5", "a.png=3..4..5", "a.png=3.5..7", "a.png=3...7",
                "a.png=3..7x5", "=3..7", "a.png=3 ..7", "a.png=٣..٧"):
        with pytest.raises(ValueError):
            cli.parse_locate(bad, ["a.png"])
        with pytest.raises(SystemExit):
            p.parse_args(common + ["--locate", bad])
    with pytest.raises(SystemExit):
        p.parse_args(common + ["--locate", "c.png=3..7"])                                # not among --suspects
    with pytest.raises(SystemExit):
        p.parse_args(common + ["--locate", "a.png=3..7", "--place", "a.png=1,2"])        # both placed and located
    f = api.Located(api.Placement(3, 5, 600, 430), 958812, 958812 / (600 * 430))
    assert cli.located_text(f, True) == "3,5 as 600x430 (mean luma difference 3.72)"
    assert cli.located_text(f, False) == "3,5 (mean luma difference 3.72)"               # entries of known size: the line of before
